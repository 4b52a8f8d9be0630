"""fp64 restatement of ``wgnn_knn_segments`` (``include/wgnn.h``) on top of ``knn_reference``, the fixtures of the batch-balanced
kNN tests, and two loop restatements of LISI.

The search: the squared distances of float32 rows in float64 (``knn_reference.sq_distances``); per segment a STABLE argsort over
the segment's members in ascending row id - equal distances go to the lower row id - with the query itself and every NaN
distance left out, short lists padded with -1 / +inf; the merged list is the union of a row's lists ordered by (distance, row
id), the -1 entries last.  The error bound and the notion of a near-tie are ``knn_reference``'s, taken per block.

LISI (Korsunsky et al. 2019): ``lisi`` is ``NeighborGraph.lisi`` as one plain loop per cell - a fixed number of tries and no
tolerance exit; ``lisi_published`` is the published ``compute_simpson_index``' search, which stops once the entropy is within
``1e-5`` of its target or after 50 tries."""
import functools

import numpy as np

import knn_reference as R

UNEVEN_SIZES = (1, 0, 63, 64, 69)                         # sums to knn_reference.LATTICE_N; one cell, no cell, a tile less one,
                                                          # a tile, a tile and a tail


def segments(x: np.ndarray, group: np.ndarray, n_groups: int, k: int):
    """``(idx int64 [n, S, k], d2 float64 [n, S, k], merged_idx int64 [n, S * k], merged_d2 float64 [n, S * k])``."""
    n = x.shape[0]
    d = R.sq_distances(x, x)
    d[np.arange(n), np.arange(n)] = np.nan
    idx = np.full((n, n_groups, k), -1, np.int64)
    d2 = np.full((n, n_groups, k), np.inf, np.float64)
    for s in range(n_groups):
        members = np.flatnonzero(np.asarray(group) == s)                          # ascending row id
        ds = d[:, members]
        take = np.argsort(ds, axis=1, kind="stable")[:, :min(k, len(members))]    # NaN sorts last
        idx[:, s, :take.shape[1]] = members[take]
        d2[:, s, :take.shape[1]] = np.take_along_axis(ds, take, axis=1)
    gone = np.isnan(d2)
    idx[gone], d2[gone] = -1, np.inf
    return (idx, d2) + merge(idx, d2)


def merge(idx: np.ndarray, d2: np.ndarray):
    """The blocked lists ``[n, S, k]`` as one list per row ``[n, S * k]``: by (d2, id) ascending, the -1 entries last."""
    n = idx.shape[0]
    flat_i, flat_d = idx.reshape(n, -1), d2.reshape(n, -1)
    m_idx, m_d2 = np.empty_like(flat_i), np.empty_like(flat_d)
    for i in range(n):
        none = flat_i[i] < 0
        order = np.lexsort((flat_i[i], flat_d[i], none))                          # the last key is the first compared
        m_idx[i], m_d2[i] = flat_i[i][order], flat_d[i][order]
    return m_idx, m_d2


def near_ties(x: np.ndarray, group: np.ndarray, n_groups: int, k: int) -> np.ndarray:
    """Boolean [n, S, k]: positions of a block whose fp64 gap to an ADJACENT distance of the same block - the (k+1)-th
    included - is below ``2 gamma d``: the kernel may list another row of the segment there."""
    _, d, _, _ = segments(x, group, n_groups, k + 1)
    g = 2.0 * R.gamma(x.shape[1])
    with np.errstate(invalid="ignore"):
        close = (d[:, :, 1:] - d[:, :, :-1]) < g * d[:, :, 1:]                    # inf - inf = NaN: False
    out = np.zeros(d.shape[:2] + (k,), bool)
    out |= close[:, :, :k]
    out[:, :, 1:] |= close[:, :, :k - 1]
    return out


@functools.lru_cache(maxsize=None)
def uneven_groups() -> np.ndarray:
    """int64 [197]: segments of ``UNEVEN_SIZES`` dealt over the rows by a fixed permutation, so that ``order`` is a real one."""
    ids = np.repeat(np.arange(len(UNEVEN_SIZES)), UNEVEN_SIZES)
    out = np.empty(R.LATTICE_N, np.int64)
    out[np.random.default_rng(17).permutation(R.LATTICE_N)] = ids
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def random_groups(n: int, n_groups: int, seed: int) -> np.ndarray:
    out = np.random.default_rng(100 + seed).integers(0, n_groups, size=n).astype(np.int64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str, n_groups: int, k: int, *case):
    """The reference lists of a fixture (computed once): ``"lattice"`` (``D``; group = row % n_groups), ``"uneven"`` (``D``) and
    ``"real"`` (``N, D, seed``; random groups) - ``(group, idx, d2, merged_idx, merged_d2)``."""
    if name == "lattice":
        x, group = R.lattice(*case), np.arange(R.LATTICE_N) % n_groups
    elif name == "uneven":
        x, group = R.lattice(*case), uneven_groups()
    else:
        x, group = R.real(*case), random_groups(case[0], n_groups, case[2])
    out = (group,) + segments(x, group, n_groups, k)
    for a in out:
        a.setflags(write=False)
    return out


def _entropy(D, beta):
    """``(H, P, sum P)`` of one cell at ``beta``: the sums run in list order."""
    P = np.exp(-D * beta)
    total, weighted = 0.0, 0.0
    for j in range(len(D)):
        total, weighted = total + P[j], weighted + D[j] * P[j]
    return np.log(total) + beta * weighted / total, P, total


def lisi(indices, distances, labels, perplexity, n_labels, tries=64, tol=None) -> np.ndarray:
    """float64 [B]: LISI by one loop per cell.  ``tol`` = None: ``tries`` tries, always; else the published exit."""
    indices, distances, labels = np.asarray(indices), np.asarray(distances, np.float64), np.asarray(labels, np.int64)
    out = np.full(indices.shape[0], np.nan)
    target = np.log(perplexity)
    for i in range(indices.shape[0]):
        js = [j for j in range(indices.shape[1]) if indices[i, j] >= 0 and np.isfinite(distances[i, j])]
        if len(js) < 2:
            continue
        D = distances[i, js] - distances[i, js].min()
        beta, low, high = 1.0, -np.inf, np.inf
        H, P, total = _entropy(D, beta)
        n = 0
        while n < tries and (tol is None or abs(H - target) > tol):
            if H > target:
                low = beta
                beta = beta * 2.0 if np.isinf(high) else (beta + high) / 2.0
            else:
                high = beta
                beta = beta / 2.0 if np.isinf(low) else (beta + low) / 2.0
            H, P, total = _entropy(D, beta)
            n += 1
        share = [0.0] * n_labels
        for j, p in zip(js, P):
            if labels[indices[i, j]] >= 0:
                share[labels[indices[i, j]]] += p
        simpson = 0.0
        for l in range(n_labels):
            s = share[l] / total
            simpson = simpson + s * s
        if simpson > 0:
            out[i] = 1.0 / simpson
    return out


def lisi_published(indices, distances, labels, perplexity, n_labels) -> np.ndarray:
    return lisi(indices, distances, labels, perplexity, n_labels, tries=50, tol=1e-5)
