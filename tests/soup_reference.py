"""numpy / Python-integer restatement of ``wgnn_soup_rows_count`` / ``wgnn_soup_rows_fill`` (``ops.soup_rows``), written from the
contract in ``include/wgnn.h``, and the cases the CPU and GPU tests share - a helper, not a test module.  Nothing here imports
torch or the package.

    sk    = mix64(key(seed, row0 + r, draw0 + d) + K_SOUP)            (uint64, wrap-around)
    u_t   = mix64(sk + t * K_READ),  t in [0, n_add[r])
    x_t   = (u_t * W) >> 64                                            (Python integers: the exact 128-bit product)
    bin_t = the k with cdf[k] <= x_t < cdf[k + 1];   s(g) = #{t : bin_t == g}
    c(g)  = cnt_r(g) + s(g);   total = lib[r] + n_add[r]
    v     = float32(log1p(float64(c) / float64(total) * scale))        - ``lognorm_reference._value``, imported, not copied
    (g, v) leaves iff c > 0 and v > threshold, in ascending g;  total == 0 gives the empty row.

What a comparison may ask is what tests/lognorm_reference.py says of a value: the float32 bits are EQUAL wherever the fp64 value
is not ``fragile``, one float32 ulp apart at most there.  Counts, bins and totals are integers: equal."""
import functools
from types import SimpleNamespace

import numpy as np

import stability_reference as R
from lognorm_reference import _value, fragile          # noqa: F401  (fragile is re-exported for the tests)
from thin_reference import K_READ, mix64_np

K_SOUP = 0x94D049BB133111EB
SCALE = 1e4
THRESHOLDS = (0.0, 1.5)
MAX_ADD = 2 ** 23
FRAGILE_CAP = 0.001


# ------------------------------------------------------------------------------------------------
# the draws
# ------------------------------------------------------------------------------------------------
def soup_key(seed: int, cell: int, draw: int) -> int:
    """``sk`` of the unit (cell, draw): the dropout block's key, moved onto a stream of its own."""
    key = (seed & R.M64) ^ ((cell * R.K_CELL) & R.M64) ^ ((draw * R.K_DRAW) & R.M64)
    return int(mix64_np(np.uint64((key + K_SOUP) & R.M64)))


def draws(seed: int, cell: int, draw: int, n_add: int, cdf) -> np.ndarray:
    """int64 [n_add]: the bin of every soup read of the unit, in read order."""
    cdf = np.asarray(cdf, np.uint64)
    W = int(cdf[-1])
    t = np.arange(int(n_add), dtype=np.uint64)
    with np.errstate(over="ignore"):
        u = mix64_np(np.uint64(soup_key(seed, cell, draw)) + t * np.uint64(K_READ))
    x = np.asarray([(int(v) * W) >> 64 for v in u], np.uint64)
    return np.searchsorted(cdf[1:], x, side="right").astype(np.int64)          # the boundaries in [1, G + 1] that are <= x


def _unit_counts(m, r, bins, G):
    """{gene: c} of one unit, and its ``s_rest``."""
    summed = {}
    for e in range(int(m.rowptr[r]), int(m.rowptr[r + 1])):
        x = float(m.cnt[e])
        if 1 <= x <= MAX_ADD:                                                  # any other value is left out
            summed[int(m.col[e])] = summed.get(int(m.col[e]), 0) + int(x)
    s = np.bincount(bins, minlength=G + 1)
    for g in np.flatnonzero(s[:G]):
        summed[int(g)] = summed.get(int(g), 0) + int(s[g])
    return summed, int(s[G])


def soup_rows(m, n_add, cdf, n_draws, threshold, seed=0, row0=0, draw0=0, scale=SCALE):
    """The contaminated rows of every unit ``q = r * n_draws + d`` as a namespace: ``rowptr`` int64 [units + 1], ``col`` int32,
    ``val`` float32, ``v64`` (the kept values before their rounding), ``cnt`` int64, ``n_out`` and ``soup_mapped`` int32 [units]."""
    G = len(cdf) - 2
    thr = np.float32(threshold)
    out_ptr, out_col, out_cnt, v64, mapped = [0], [], [], [], []
    for r in range(len(m.rowptr) - 1):
        for d in range(n_draws):
            bins = draws(seed, row0 + r, draw0 + d, int(n_add[r]), cdf)
            summed, s_rest = _unit_counts(m, r, bins, G)
            total = int(m.lib[r]) + int(n_add[r])
            mapped.append(int(n_add[r]) - s_rest)
            for g in sorted(summed):
                c = summed[g]
                if total > 0 and c > 0:
                    v = _value(float(c), float(total), scale)
                    if np.float32(v) > thr:
                        out_col.append(g); out_cnt.append(c); v64.append(v)
            out_ptr.append(len(out_col))
    v64 = np.asarray(v64, np.float64)
    rowptr = np.asarray(out_ptr, np.int64)
    return SimpleNamespace(rowptr=rowptr, col=np.asarray(out_col, np.int32), val=v64.astype(np.float32), v64=v64,
                           cnt=np.asarray(out_cnt, np.int64), n_out=np.diff(rowptr).astype(np.int32),
                           soup_mapped=np.asarray(mapped, np.int32))


def contaminated_dense(m, n_add, cdf, n_draws, seed=0, row0=0, draw0=0):
    """The units' contaminated counts as a dense float32 ``[units, G + 1]`` matrix - the last column holds the cell's reads outside
    the bundle plus ``s_rest`` - and the int32 gene map that sends column ``g`` to gene ``g`` and the last one to -1: what
    ``align_rows(..., normalize="lognorm")`` takes.  Exact while every entry is <= 2^24."""
    G = len(cdf) - 2
    B = len(m.rowptr) - 1
    dense = np.zeros((B * n_draws, G + 1), np.float64)
    for r in range(B):
        for d in range(n_draws):
            bins = draws(seed, row0 + r, draw0 + d, int(n_add[r]), cdf)
            summed, s_rest = _unit_counts(m, r, bins, G)
            own = sum(int(x) for x in m.cnt[m.rowptr[r]:m.rowptr[r + 1]] if 1 <= x <= MAX_ADD)
            row = dense[r * n_draws + d]
            for g, c in summed.items():
                row[g] = c
            row[G] = int(m.lib[r]) - own + s_rest
    assert dense.max() <= 2 ** 24
    return dense.astype(np.float32), np.concatenate([np.arange(G), [-1]]).astype(np.int32)


def cdf_of(weights) -> np.ndarray:
    """uint64 [len(weights) + 1]: the cumulative weights, from 0."""
    out = np.zeros(len(weights) + 1, np.uint64)
    out[1:] = np.cumsum(np.asarray(weights, np.uint64), dtype=np.uint64)
    return out


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
G_CASE = 300
N_DRAWS = 3
CASE_SEED = 0x5009
ONE_GENE = 123
(ROW_EMPTY, ROW_PURE_SOUP, ROW_FOREIGN_ONLY, ROW_ONE, ROW_63, ROW_64, ROW_65, ROW_ALL, ROW_UNSORTED, ROW_TWICE, ROW_DEEP_A, ROW_DEEP_B,
 ROW_DEEP_C, ROW_513) = range(14)
N_ADD = (0, 40, 1, 1, 63, 64, 65, 513, 64, 63, 3000, 3000, 3000, 513)
DEEP_ROWS = (ROW_DEEP_A, ROW_DEEP_B, ROW_DEEP_C)


@functools.lru_cache(maxsize=None)
def batch():
    """The count batch of the soup tests over ``G_CASE`` genes: an empty row that takes no soup, an empty row that takes 40 reads
    (a pure-soup droplet), an empty row with reads outside the bundle, rows of 1 / 63 / 64 / 65 / 300 genes (the last one holds a
    count of 2^23), a row in descending order, a row that lists gene 7 twice and gene 299 three times, three random rows that
    take 3000 reads and one that takes 513.  ``lib`` = the row's sum plus, on every third row, reads outside the bundle;
    ``n_add`` = ``N_ADD``."""
    rng = np.random.default_rng(61_000)
    pick = lambda n: np.sort(rng.choice(G_CASE, size=n, replace=False))
    rows = [np.zeros(0, int), np.zeros(0, int), np.zeros(0, int), np.array([5]), pick(63), pick(64), pick(65), np.arange(G_CASE),
            np.arange(290, 10, -7), np.array([7, 120, 7, 299, 299, 3, 299]), pick(150), pick(40), pick(220), pick(90)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    cnt = rng.geometric(0.4, col.shape[0]).astype(np.float32)
    cnt[rowptr[ROW_ALL] + 11] = 2.0 ** 23                               # the largest count the operand check admits
    rest = np.where(np.arange(len(rows)) % 3 == 0, rng.integers(1, 4000, len(rows)), 0)
    rest[ROW_EMPTY], rest[ROW_PURE_SOUP], rest[ROW_FOREIGN_ONLY] = 0, 0, 7
    lib = np.asarray([cnt[rowptr[r]:rowptr[r + 1]].sum() for r in range(len(rows))], np.int64) + rest
    return SimpleNamespace(rowptr=rowptr, col=col, cnt=cnt, lib=lib, rest=rest, B=len(rows), G=G_CASE,
                           n_add=np.asarray(N_ADD, np.int64))


@functools.lru_cache(maxsize=None)
def profiles():
    """{name: cdf uint64 [G + 2]}: ``uniform`` (weight 5 on two genes of three, none on the third, 50 on the rest bin), ``one``
    (everything on ``ONE_GENE``), ``rest`` (everything outside the bundle), ``wide`` (weights up to 2^40, a few tiny ones among
    them: W > 2^48, so the high multiply needs all 64 bits of the hash)."""
    G = G_CASE
    rng = np.random.default_rng(61_001)
    uniform = np.where(np.arange(G + 1) % 3 == 1, 0, 5)
    uniform[G] = 50
    one = np.zeros(G + 1, np.int64)
    one[ONE_GENE] = 17
    rest = np.zeros(G + 1, np.int64)
    rest[G] = 9
    wide = 2 ** 40 - rng.integers(0, 2 ** 36, G + 1)
    wide[[3, 150, 298]] = (1, 2, 1000)
    wide[[4, 77]] = 0
    return dict(uniform=cdf_of(uniform), one=cdf_of(one), rest=cdf_of(rest), wide=cdf_of(wide))


@functools.lru_cache(maxsize=None)
def case(profile: str, threshold: float):
    """The batch, a profile and the reference's contaminated rows at ``threshold``."""
    m = batch()
    cdf = profiles()[profile]
    return SimpleNamespace(m=m, cdf=cdf, threshold=threshold, ref=soup_rows(m, m.n_add, cdf, N_DRAWS, threshold, seed=CASE_SEED))
