"""fp64 brute-force restatement of ``wgnn_knn_rows`` (``include/wgnn.h``), its error bound, and the fixtures of the kNN tests.

The reference takes the squared Euclidean distances of float32 rows in float64 (``((Q[:, None] - X[None])**2).sum(-1)``), orders
each query's candidates by a STABLE argsort - equal distances go to the lower index - leaves the query itself and every NaN
distance out, and pads short lists with -1 / +inf.

The kernel's distance is a chain of D ``fmaf(t, t, d)`` over f32 differences ``t``: every term is non-negative, so the standard
bound of a length-D sum plus one rounding for the difference (squared: two) and one for the product gives
``|d - exact| <= gamma * exact`` with ``gamma = (D + 3) u / (1 - (D + 3) u)``, ``u = 2^-24`` (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1).  Two distances closer than ``2 gamma d`` may therefore legitimately swap: a NEAR-TIE."""
import functools

import numpy as np

U = 2.0 ** -24
LATTICE_N, LATTICE_DIMS = 197, (20, 36, 256)
REAL_CASES = ((300, 20, 0), (300, 200, 0), (197, 36, 1))          # (N, D, seed)
TINY_N, TINY_K = 10, 15


def gamma(D: int) -> float:
    return (D + 3) * U / (1.0 - (D + 3) * U)


def sq_distances(queries: np.ndarray, x: np.ndarray) -> np.ndarray:
    """float64 [n_q, n_c]: the exact-in-fp64 squared distances of float32 rows (row by row: no [n_q, n_c, D] array)."""
    q, c = np.asarray(queries, np.float64), np.asarray(x, np.float64)
    out = np.empty((q.shape[0], c.shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(q.shape[0]):
            out[i] = ((q[i][None, :] - c) ** 2).sum(-1)
    return out


def knn(x: np.ndarray, k: int, queries=None, self_offset=0):
    """``(idx int64 [n_q, k], d2 float64 [n_q, k])``: per query the k candidates smallest under (distance, index);
    ``self_offset`` = None: no candidate is left out, else query i is candidate ``self_offset + i``."""
    q = x if queries is None else queries
    d = sq_distances(q, x)
    if self_offset is not None:
        d[np.arange(q.shape[0]), self_offset + np.arange(q.shape[0])] = np.nan
    order = np.argsort(d, axis=1, kind="stable")                  # NaN sorts last
    idx = np.full((q.shape[0], k), -1, np.int64)
    d2 = np.full((q.shape[0], k), np.inf, np.float64)
    n = min(k, x.shape[0])
    idx[:, :n] = order[:, :n]
    d2[:, :n] = np.take_along_axis(d, order[:, :n], axis=1)
    gone = np.isnan(d2)
    idx[gone], d2[gone] = -1, np.inf
    return idx, d2


def near_ties(x: np.ndarray, k: int, queries=None, self_offset=0) -> np.ndarray:
    """Boolean [n_q, k]: list positions whose fp64 gap to an ADJACENT distance - the (k+1)-th included - is below
    ``2 gamma d``: the kernel may list another candidate there."""
    _, d = knn(x, k + 1, queries, self_offset)
    g = 2.0 * gamma(x.shape[1])
    with np.errstate(invalid="ignore"):
        close = (d[:, 1:] - d[:, :-1]) < g * d[:, 1:]             # between positions j and j + 1; inf - inf = NaN: False
    out = np.zeros((d.shape[0], k), bool)
    out |= close[:, :k]
    out[:, 1:] |= close[:, :k - 1]
    return out


@functools.lru_cache(maxsize=None)
def lattice(D: int) -> np.ndarray:
    """float32 [197, D]: multiples of 1/8 in [-4, 4]; rows 50 and 120 are copies of row 7, row 121 of row 8.  Every squared
    distance is an integer multiple of 2^-6 below 2^18 of them: a float32 sum in any order is exact."""
    assert D in LATTICE_DIMS
    x = (np.random.default_rng(3).integers(-32, 33, size=(LATTICE_N, D)) / 8.0).astype(np.float32)
    x[50], x[120], x[121] = x[7], x[7], x[8]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def real(N: int, D: int, seed: int) -> np.ndarray:
    x = np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tiny() -> np.ndarray:
    x = np.random.default_rng(5).standard_normal((TINY_N, 8)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name: str, k: int, *case):
    """The reference lists of a fixture (computed once): ``reference("lattice", 15, 36)``, ``reference("real", 15, 300, 20, 0)``."""
    x = {"lattice": lattice, "real": real, "tiny": tiny}[name](*case)
    idx, d2 = knn(x, k)
    idx.setflags(write=False); d2.setflags(write=False)
    return idx, d2
